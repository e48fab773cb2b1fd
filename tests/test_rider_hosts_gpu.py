"""GPU: every rider kind and every rider-hosting kernel form at kernel level (csrc/rider_dev.h, csrc/pair.hip, the `_r` launchers of
csrc/pointmlp.hip), bit for bit against the stand-alone launches -- the cases of tests/rider_check.py, which
tests/test_rider_hosts_cpu.py validates on the specification library.  Each comparison uses separate, sentinel-filled, guarded buffers
for the three runs (stand-alone launches, the set alone, the set inside its host) and checks the barrier words after three repetitions."""
import pytest

import rider_check as rc
from fake_t3d import FakeLib
from transferable3d_amd import abi

pytestmark = pytest.mark.gpu

# rider-op shapes tests/test_kernels_gpu.py pins against the oracle already: none of the shapes of part A (its FC layers are
# 128..1024 -> 3..512 at B in {8, 32, 64, 128}, its finalizers N = 192 and 64..256 at >= 640 tiles), so every case is also compared
# with the fp64 specification at the tolerance of the existing test of its kernel (rider_check.ORACLE_TOL).


SPEC = rc.Env(FakeLib(), 'cpu')


@pytest.fixture
def env(hip_lib):
    return rc.Env(hip_lib, 'cuda')


# ---- A ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id,factory,args', rc.KIND_CASES, ids=[c[0] for c in rc.KIND_CASES])
def test_each_rider_kind_as_a_set_of_its_own(env, case_id, factory, args):
    case = factory(*args)
    rs = rc.check_set_alone(env, case, what=case_id)
    blocks = {'bn_fwd': lambda: -(-args[0] // rc.FC_CH), 'bn_bwd': lambda: -(-args[0] // rc.FC_CH), 'fc_fwd': lambda: -(-args[2] // rc.CB),
              'fc_bwd': lambda: -(-args[2] // rc.CB), 'fc_dinput': lambda: -(-args[2] // rc.CB), 'dy_colsum': lambda: -(-args[0] * args[1] // 256)}
    assert rs.n_ops == 1 and rs.n_wg == min(blocks[case_id.split('-')[0]](), rc.RIDER_MAX_WG), rs.n_wg
    rc.check_against_oracle(env, SPEC, case, case_id)


@pytest.mark.parametrize('M,K,N,rpf', rc.MID_SHAPES)
def test_wide_rider_pool_bwd_mid(env, M, K, N, rpf):
    rc.check_wide_rider(env, M, K, N, rpf)
    N = N if rc.sparse_rows_lds(N) <= 76 * 1024 else 512
    rc.check_against_oracle(env, SPEC, rc.pool_bwd_mid_case(M, K, N, rpf), 'pool_bwd_mid')


# ---- B ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_ops', [abi.RIDER_MAX_OPS, 2])
def test_dependent_chain_of_mixed_kinds(env, n_ops):
    rs = rc.check_set_alone(env, rc.fc_head_bwd_case(n_ops), what='head backward, %d ops' % n_ops)
    assert rs.n_wg == (rc.RIDER_MAX_WG if n_ops > 2 else 8)      # 64- and 128-block ops on 32 workgroups; 3 and 8 blocks on 8
    if n_ops > 2:
        rc.check_against_oracle(env, SPEC, rc.fc_head_bwd_case(n_ops), 'head backward')


@pytest.mark.parametrize('pattern', [(0, 0, 0, 0), (0, 1, 0, 1)], ids=['independent', '0101'])
def test_hand_built_sets_without_barriers(env, pattern):
    rc.check_set_alone(env, rc.independent_case(pattern), depends=list(pattern), what='depends=%s' % (pattern,))
    rc.check_against_oracle(env, SPEC, rc.independent_case(pattern), 'depends=%s' % (pattern,))


def test_fc_chain_ops_against_the_oracle(env):
    """The 4-op FC chain every host row carries (tests/test_riders_gpu.py `_fc_chain`: 256 -> 512 -> 512 -> 256 -> 64 at B = 32) and the
    two-op chain of the non-hosting rows: their layers, one launch each, against the fp64 specification."""
    rc.check_against_oracle(env, SPEC, rc.fc_chain_case(**rc.FC_CHAIN), 'fc chain')
    rc.check_against_oracle(env, SPEC, rc.small_chain_case(), 'small chain')


# ---- C ----------------------------------------------------------------------------------------------------------------------------------
REACHABLE = [f for f in rc.HOST_FORMS if not f.unreachable]


@pytest.mark.parametrize('form', REACHABLE, ids=[f.id for f in REACHABLE])
def test_every_hosting_form(env, monkeypatch, form):
    """One row of rider_check.HOST_FORMS: the library confirms that these arguments host, with the row's arithmetic and tiles; then the
    host with riders == NULL, the FC chain alone and the `_r` call with the chain, three repetitions each, bit for bit."""
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)
    rc.check_form(env, form)


WIDE_ROWS = rc.FAMILY_ROWS + ['k_pointmlp_fwd_r<64, false, PathX3>', 'k_pointmlp_bwd_r<64, 64, 64, PathX3>', 'k_pool_bwd_stage1_r<64, PathX3>',
                              'k_pool_bwd_stage2_r<64, PathX3>']


@pytest.mark.parametrize('kernel', WIDE_ROWS, ids=[k.replace(' ', '') for k in WIDE_ROWS])
def test_wide_rider_inside_each_launcher_family(env, kernel):
    """t3d_pool_bwd_mid (771 workgroups, 72.5 KB of LDS) in the smallest row of each family: the launch's LDS is the rider's, and the
    host's own grid (2 to 68 tiles) is smaller than n_wg."""
    rc.check_form_with_wide_rider(env, rc.form_by_name(kernel))


# ---- D ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n[0] for n in rc.NON_HOSTING])
def test_r_call_on_a_form_that_does_not_host(env, name):
    rc.check_non_hosting(env, name, expect_query=0)


# ---- E ----------------------------------------------------------------------------------------------------------------------------------
def test_riders_plan_refusals(env):
    rc.check_plan_refusals(env)


def test_run_riders_and_r_launcher_refusals(env):
    rc.check_launch_refusals(env)


def test_hosts_riders_queries_refuse_what_the_launchers_refuse(env):
    rc.check_query_refusals(env)
