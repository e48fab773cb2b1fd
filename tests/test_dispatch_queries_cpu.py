"""CPU: the `_hosts_riders` queries of the BUILT library (csrc/pointmlp.hip select_*) on the rows of tests/rider_check.py.  A query is the
launcher's selection step alone -- argument checks, tiles, `hosts` -- with no stream, no rider set and no HIP call, and it never reads
through a pointer argument: host tensors serve.  So the dispatch the GPU tests rely on (tests/test_rider_hosts_gpu.py) is asked of
libt3d.so before any GPU is involved: every hosting row hosts with the arithmetic and tiles it names, every non-hosting row answers 0,
and rejected arguments come back with the launcher's own error code."""
import pytest
import torch

import rider_check as rc
from transferable3d_amd import abi

REACHABLE = [f for f in rc.HOST_FORMS if not f.unreachable]


@pytest.fixture(scope='module')
def env():
    return rc.Env(abi.load(), 'cpu')


@pytest.fixture(autouse=True)
def planes_without_a_launch(monkeypatch):
    """The `pre` rows split their weights on the device (rc.x3_planes -> t3d_split_x3_frag, a launch).  A query looks at the plane
    pointer and its stride only: zeroed host planes of the same size stand in."""
    def planes(env, w):
        K, N = w.shape
        stride = (K * N + 7) // 8 * 8
        return torch.zeros(3 * stride, dtype=torch.bfloat16), torch.zeros(3 * stride, dtype=torch.bfloat16), stride
    monkeypatch.setattr(rc, 'x3_planes', planes)


@pytest.mark.parametrize('form', REACHABLE, ids=[f.id for f in REACHABLE])
def test_every_hosting_row_hosts_with_the_tiles_it_names(env, monkeypatch, form):
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)
    rc.check_form_claims(env, form, rc.form_host(env, form))


@pytest.mark.parametrize('name', [n[0] for n in rc.NON_HOSTING])
def test_query_is_zero_for_every_form_that_does_not_host(env, name):
    _, builder, kw, arith, _ = [n for n in rc.NON_HOSTING if n[0] == name][0]
    host = builder(env, arith=arith, **kw)
    _, args = host(rc.Bufs(env.dev))
    assert host.query(env.lib, args) == 0, name


def test_queries_refuse_what_the_launchers_refuse(env):
    rc.check_query_refusals(env)
