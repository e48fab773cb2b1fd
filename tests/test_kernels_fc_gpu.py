"""GPU: the three fully-connected bodies of csrc/fc_dev.h in their three launch forms (stand-alone csrc/fc.hip, rider csrc/rider_dev.h, paired
csrc/pair.hip) at their edges: the cases of tests/fc_check.py on libt3d.so, each stand-alone launch against the fp64 specification
(tests/fake_t3d.py) on identical seeded inputs with rider_check.ORACLE_TOL, every output sentinel-filled and fenced by guard bands, padding
columns of strided outputs still holding the sentinel; the rider form and the paired form bit for bit against the stand-alone launches.
tests/test_kernels_fc_cpu.py runs the same cases on the specification and holds the host-only checks (activation margins, the float32
restatement of the K = 1096 reduction, deliberately wrong libraries, the specification against autograd).

MEASURED_WORST (one run of this module on the MI355X, 494 passed in 3.4 s; against the fp64 specification, never against another run of a
kernel; per (kind, output), over the stand-alone launches of part 1 and the paired launches of part 3: the largest error, the bound at that
element in brackets, the largest `error / bound` and the case it came from.  No bound follows a measurement: they are
rider_check.ORACLE_TOL, the tolerances of tests/test_kernels_gpu.py.  The finalizers and the column sums accumulate in double: no error.
Bit-for-bit comparisons -- rider form and paired form against the stand-alone launches, padding columns, guard bands -- have no line.)
  bn_bwd     coef       0.000e+00  (1.030e-05)  0.000   bn_bwd+bn_bwd paired
  bn_bwd     dbeta      0.000e+00  (1.295e-05)  0.000   bn_bwd+bn_bwd paired
  bn_bwd     dgamma     0.000e+00  (2.287e-05)  0.000   bn_bwd+bn_bwd paired
  bn_bwd     dpool      0.000e+00  (2.267e-06)  0.000   bn_bwd+bn_bwd paired
  dy_colsum  colsum     0.000e+00  (3.633e-03)  0.000   bn_bwd+dy_colsum paired
  fc_bwd     db         3.815e-06  (1.849e-02)  0.001   bwd-form-B97-next-nobn-relu-drop op 0 t3d_fc_bwd
  fc_bwd     dbeta      3.815e-06  (1.437e-02)  0.001   fc_bwd-B128+bn_bwd-dense-T8 paired
  fc_bwd     dgamma     3.815e-06  (6.965e-03)  0.001   bwd-next-B97-Nn67 op 0 t3d_fc_bwd
  fc_bwd     dw         1.526e-05  (2.828e-02)  0.001   bwd-red-B97-K13-ld13-K2_0 op 0 t3d_fc_bwd
  fc_bwd     dy         1.192e-06  (2.982e-03)  0.000   bwd-form-B31-nobn-no-dbias op 0 t3d_fc_bwd
  fc_dinput  bn_coef    3.725e-09  (3.262e-06)  0.001   dinput-fused-B1-K96-train op 0 t3d_fc_dinput
  fc_dinput  bn_db      3.815e-06  (2.374e-03)  0.007   bn_bwd-dense-T8+fc_dinput-B128 paired
  fc_dinput  bn_dg      5.722e-06  (2.040e-03)  0.014   dinput-fused-B128-K96-train op 0 t3d_fc_dinput
  fc_dinput  din        7.153e-07  (3.733e-05)  0.040   bn_bwd-dense-T8+fc_dinput-B128 paired
  fc_dinput  dpool      5.364e-07  (1.532e-05)  0.035   bn_bwd-dense-T8+fc_dinput-B128 paired
  fc_fwd     invstd     9.537e-06  (5.908e-03)  0.003   fwd-rows-B2 op 0 t3d_fc_fwd
  fc_fwd     mean       2.384e-07  (6.742e-04)  0.001   fwd-rows-B1 op 0 t3d_fc_fwd
  fc_fwd     mm         1.192e-07  (3.949e-04)  0.000   fwd-rows-B1 op 0 t3d_fc_fwd
  fc_fwd     mv         2.384e-07  (5.394e-04)  0.001   fwd-red-B31-K72-ld72-K2_0 op 0 t3d_fc_fwd
  fc_fwd     out        1.431e-06  (1.024e-03)  0.004   fwd-red-B97-K1096-ld1096-K2_0 op 0 t3d_fc_fwd
  fc_fwd     y          9.537e-07  (5.162e-04)  0.004   fwd-red-B97-K1096-ld1096-K2_0 op 0 t3d_fc_fwd

FORM COVERAGE (mechanism -> test ids of this module)
  RBT = 1 (B <= 32) / RBT = MAXRB (B > 32), stand-alone                                                     test_fc_against_spec[*-rows-B1 .. B32], [*-rows-B33 .. B128]
  partly filled row blocks (B = 33, 65, 97, 127), B = 1 (variance 0)                                        test_fc_against_spec[*-rows-*]
  ragged last column block, one column, two blocks                                                          test_fc_against_spec[*-cols-*]
  vector k-loop only (K % 8 == 0, ld_in % 4 == 0)                                                           test_fc_against_spec[*-red-*-K8-*], [*-K72-*], [*-K1096-*], [*-rows-*]
  scalar k-loop only (ld_in & 3 != 0, or K < 8)                                                             test_fc_against_spec[*-red-*-K3-*], [*-K13-*], [*-K68-ld70-*]
  `gfull` tail: vector groups, then a half group                                                            test_fc_against_spec[*-red-*-K60-ld60-K2_0]
  a k-group straddling in | in2, ragged end at 70                                                           test_fc_against_spec[*-red-*-K60-ld60-K2_10], [*-form-*]
  vector loop at a stride that is not K, scalar groups in in2                                               test_fc_against_spec[*-red-*-K64-ld68-K2_10]
  idle waves (1 group: seven; 9 groups: waves with 2, 1, 0)                                                 test_fc_against_spec[*-red-*-K8-*], [*-K72-*]
  second GIF batch (RBT = 1: 16 groups per wave; MAXRB: 4; rider: 6)                                        test_fc_against_spec[*-red-B31-K1096-*], [*-red-B97-*], test_fc_rider_form[*-red-B31-K1096-*]
  prefetched dW (RBT = 1, blocks < 32) / looped dW (MAXRB; RBT = 1 beyond 32 blocks; rider beyond 8)        test_fc_against_spec[bwd-*-B31-*], [bwd-*-B97-*], [bwd-red-B31-K1096-*], test_fc_rider_form[bwd-red-B31-K1096-*]
  dW store guard kk < Kt, at_nb through in2                                                                 test_fc_against_spec[bwd-red-*]
  wave_gemm<true> scalar (ldw = 3, 9, 67) / vector (96) / vector then half group (100)                      test_fc_against_spec[dinput-red-*], [bwd-next-*]
  identity form (w == NULL)                                                                                 test_fc_against_spec[fwd-form-*-identity-*]
  optional pointers, activations, dropout, add_in, eval / frozen batch-norm, unbiased_ema = 0               test_fc_against_spec[*-form-*]
  fused pooled batch-norm backward of fc_dinput: training, frozen with NULL statistics, no dgamma / dbeta   test_fc_against_spec[dinput-fused-*]
  rider form (256 threads, NWP = 4, GIF = 6, XKB = 2)                                                       test_fc_rider_form
  paired form, k_small_pair<1>                                                                              test_fc_case_in_a_pair[*-B1 .. B32-*], test_small_pair[<kind>+<kind>], [blocks-*]
  paired form, k_small_pair<MAXRB>                                                                          test_fc_case_in_a_pair[*-B33 .. B128-*], test_small_pair[*-B33*], [*-B128*]
  k_small_pair without an FC op (rows = 0)                                                                  test_small_pair[dy_colsum+dy_colsum], [bn_bwd+bn_bwd], [bn_bwd+dy_colsum], [dy_colsum+bn_bwd]
  blockIdx.x < n_a split: 1 block beside 64, both orders; ragged N = 67 on both sides                       test_small_pair[blocks-*]
  frozen bn_bwd_finalize with gamma = mean = invstd = NULL                                                  test_bn_bwd_frozen_with_null_statistics, test_small_pair[*frozen-null-stats*]
  refusals of t3d_fc_fwd / t3d_fc_bwd / t3d_fc_dinput / t3d_small_pair                                      test_fc_refusals, test_fc_null_struct, test_small_pair_refusals
"""
import pytest

import fc_check as fc

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(hip_lib):
    return fc.Env(hip_lib, 'cuda')


# ---- 1. the FC kernels at their edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.CASE_IDS)
def test_fc_against_spec(env, cid):
    fc.check_case(env, cid, fc.STATS)


@pytest.mark.parametrize('rid', fc.REFUSAL_IDS)
def test_fc_refusals(env, rid):
    fc.check_refusal(env, rid)


def test_fc_null_struct(env):
    fc.check_null_struct(env)


# ---- 2. the rider form ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.RIDER_IDS)
def test_fc_rider_form(env, cid):
    fc.check_rider(env, cid)


# ---- 3. t3d_small_pair ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.PAIRED_IDS)
def test_fc_case_in_a_pair(env, cid):
    fc.check_case_in_a_pair(env, cid)


@pytest.mark.parametrize('pid', fc.PAIR_IDS)
def test_small_pair(env, pid):
    fc.check_pair_id(env, pid, fc.STATS)


@pytest.mark.parametrize('rid', fc.PAIR_REFUSAL_IDS)
def test_small_pair_refusals(env, rid):
    fc.check_pair_refusal(env, rid)


@pytest.mark.parametrize('dense', [1, 0])
def test_bn_bwd_frozen_with_null_statistics(env, dense):
    fc.check_bn_bwd_frozen(env, dense, fc.STATS)

