"""GPU: tests/test_boxpc_rep_b_cpu.py -- the Box-PC Fit net's representation B in stage b, stage c and the inference graph -- re-run
with the HIP library on the MI355X under both GEMM arithmetics, plus a full-size stage-b trajectory, a bf16 step and two hipGraph replays
from one state."""
import numpy as np
import pytest
import torch

import ref_boxpc_b as RB
import test_boxpc_rep_b_cpu as T
from model_check import trajectory_check
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

ARITHS = ['bf16x3', 'fp32_mfma']


@pytest.fixture(params=ARITHS)
def hip_rt(request, hip_lib, monkeypatch):
    monkeypatch.setattr(T, '_runtime', lambda: Runtime(lib=hip_lib, gemm_arithmetic=request.param))
    monkeypatch.setattr(T, 'SHAPE', (8, 256))
    return request.param


@pytest.mark.parametrize('one_hot', [False, True])
def test_stage_b_trajectory_follows_the_oracle(hip_rt, monkeypatch, one_hot):
    T.test_stage_b_trajectory_follows_the_oracle(monkeypatch, one_hot)


@pytest.mark.parametrize('n_refine,min_fit', [(1, False), (1, True), (2, False), (2, True)])
def test_stage_c_trajectory_follows_the_oracle(hip_rt, monkeypatch, n_refine, min_fit):
    T.test_stage_c_trajectory_follows_the_oracle(monkeypatch, n_refine, min_fit)


@pytest.mark.parametrize('mask_pc', [False, True])
def test_inference_graph_refines_with_representation_b(hip_rt, monkeypatch, mask_pc):
    T.test_inference_graph_refines_with_representation_b(monkeypatch, mask_pc)


def test_stage_c_backward_has_no_per_point_launch_for_the_boxpc_branch(hip_rt):
    T.test_stage_c_backward_has_no_per_point_launch_for_the_boxpc_branch()


def test_point_branch_is_emitted_once_for_every_evaluation(hip_rt):
    T.test_point_branch_is_emitted_once_for_every_evaluation()


def test_shared_point_branch_is_bit_identical_to_one_per_evaluation(hip_rt, monkeypatch):
    T.test_shared_point_branch_is_bit_identical_to_one_per_evaluation(monkeypatch)


@pytest.mark.parametrize('one_hot', [False, True])
def test_reference_call_sequence_of_get_model(hip_rt, one_hot):
    T.test_reference_call_sequence_of_get_model(one_hot)


def test_full_size_stage_b_trajectory(hip_lib, monkeypatch):
    """B = 32, N = 1024, C = 4: the shape tools/bench_boxpc_rep.py times."""
    RB.use_rep_b(monkeypatch)
    rep = trajectory_check(Runtime(lib=hip_lib), 'boxpc', steps=2, B=32, N=1024, C=4, config_over=dict(T.BOXPC_B))
    assert all(r['weight_entries_checked'] > 1000 for r in rep[:-1])


@pytest.mark.parametrize('workload', ['boxpc', 'F'])
def test_bf16_steps_stay_close_to_fp32_and_train(hip_lib, workload):
    """Representation B with dtype = bf16, the bounds of tests/test_bf16_gpu.py's stage-b / stage-c wiring check: first loss within 3 % /
    8 % of the fp32 step on the same weights and batch, finite and decreasing over 8 steps on a fixed batch, a second run bit-identical."""
    from transferable3d_amd.step import build_training_step
    from transferable3d_amd.synthetic import make_batch
    B, N, C = 32, 1024, 4
    flags = T._stage_b_flags() if workload == 'boxpc' else T._stage_c_flags()
    runs = {}
    for dtype, rep in (('f32', 0), ('bf16', 0), ('bf16', 1)):
        g, model, step, loss = build_training_step(Runtime(lib=hip_lib), workload, B, N, C, dtype=dtype, seed=11, c=flags)
        model.inputs.load(make_batch(B, N, C, seed=5, boxpc=(workload == 'boxpc')))
        cur = []
        for k in range(8):
            step.run()
            cur.append(float(loss))
        torch.cuda.synchronize()
        runs[(dtype, rep)] = (cur, g.vars.params[:g.vars.used].clone())
    f32, b0, b1 = runs[('f32', 0)], runs[('bf16', 0)], runs[('bf16', 1)]
    assert all(np.isfinite(b0[0])) and b0[0][-1] < b0[0][0], b0[0]
    assert abs(b0[0][0] - f32[0][0]) < (3e-2 if workload == 'boxpc' else 8e-2) * abs(f32[0][0]), (b0[0][0], f32[0][0])
    assert b0[0] == b1[0] and torch.equal(b0[1], b1[1])


@pytest.mark.parametrize('workload', ['boxpc', 'F'])
def test_two_graph_replays_from_one_state_are_bit_identical(hip_lib, workload):
    from transferable3d_amd.step import build_training_step
    from transferable3d_amd.synthetic import make_batch
    B, N, C = 8, 256, 4
    flags = T._stage_b_flags() if workload == 'boxpc' else T._stage_c_flags(2, True)
    g, model, step, loss = build_training_step(Runtime(lib=hip_lib), workload, B, N, C, seed=3, c=flags, use_hip_graph=True)
    model.inputs.load(make_batch(B, N, C, seed=7, boxpc=(workload == 'boxpc')))
    step.run()                                          # (eager)
    step.run()                                          # (capture + first replay)
    torch.cuda.synchronize()
    vs = g.vars
    state = [t.clone() for t in (vs.params, vs.state, vs.adam_m, vs.adam_v, g.hyper)]
    outs = []
    for _ in range(2):
        for t, s in zip((vs.params, vs.state, vs.adam_m, vs.adam_v, g.hyper), state):
            t.copy_(s)
        torch.cuda.synchronize()
        step.run()
        torch.cuda.synchronize()
        outs.append([float(loss)] + [t.clone() for t in (vs.params, vs.state, vs.grads)])
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)
