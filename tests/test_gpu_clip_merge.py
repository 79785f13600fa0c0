"""The merged clip passes of the camera stage (tc_clip.h, cam_group_regs) on the GPU: frames through tc_step and through
one tc_step_multi call against the oracle's, bit for bit, with TC_CLIP_MERGE=1 (default) and 0 (always four passes).

simple_layout runs the single-group register path of the K = 5 kernels; stress_graph the same kernels on a graph with
hubs and shared targets.  Env 0 of the simple_layout case is parked (zero velocity, zero action: the pose does not
move) at a pose the CPU study found NOT mergeable for passes 1+2 -- two straddling edges share a target -- so the
refusal and the literal fallback are on the path next to frames that do merge; the CPU form of the pair test
(tests/test_clip_merge_cpu.py) says which frames of the run are which.

What this test cannot see is WHICH form the kernel took for a frame: merged and literal passes give the same frame by
construction, and the merged / refused counts asserted below come from the CPU form of the test.  The kernels carry no
counter for it (an atomic per frame in a kernel that is short of scalar registers).
"""
import numpy as np
import pytest

import orc
from test_clip_merge_cpu import ClipStage, build_shim
from test_gpu_parity import make_env, make_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, K = 16, 6
# simple_layout, from the CPU study (bench.py's action distribution): passes 1+2 refused, passes 3+4 merged
PARKED = (1.2266666688791368, 1.5243333333333628, -1.570756502325519)


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("tc_clip_gpu"))


def _start(map_name, park):
    """env and oracle after the same reset; env 0 parked at PARKED through load_state_dict"""
    env = make_env(map_name, "r64", "classes", N)
    o = make_oracle(env)
    env.reset(seed=5)
    o.reset(env._keep[0].cpu().numpy())
    if park:
        sd = env.state_dict()
        for k, v in zip(("x", "y", "theta", "velocity", "steering"), PARKED + (0.0, 0.0)):
            sd["state"][k][0] = v
            o.state[k][0] = v
        env.load_state_dict(sd)
    return env, o


def _actions(park):
    rng = np.random.default_rng(2)
    cc = np.stack([rng.uniform(0.3, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2).astype(np.float32)
    if park:
        cc[:, 0, :] = 0.0
    man = rng.integers(0, 4, (K, N)).astype(np.int32)
    return cc, man


def _count(stage, o, total):
    """the pair test's answers for the oracle's current poses, added to total[8]; -> env 0's"""
    first = None
    for i in range(N):
        s = o.state[i]
        _, _, cnt = stage.capture(float(s["x"]), float(s["y"]), float(s["theta"]))
        total += cnt
        first = cnt if first is None else first
    return first


@pytest.mark.parametrize("merge", ["1", "0"])
@pytest.mark.parametrize("map_name", ["simple_layout", "stress_graph"])
def test_frames_equal_the_oracle(map_name, merge, shim, monkeypatch):
    monkeypatch.setenv("TC_CLIP_MERGE", merge)
    park = map_name == "simple_layout"
    stage = ClipStage(shim, map_name)
    cc, man = _actions(park)
    total = np.zeros(8, dtype=np.int64)

    env, o = _start(map_name, park)  # K x tc_step
    for k in range(K):
        env.step({"car_control": cc[k], "maneuver": man[k]})
        o.step(cc[k].astype(np.float64), man[k])
        torch.cuda.synchronize()
        g = env.out["obs"].cpu().numpy().reshape(N, -1)
        bad = np.flatnonzero((g != o.obs).any(axis=1))
        assert bad.size == 0, ("tc_step", map_name, merge, "step", k, "envs", bad[:8])
        env0 = _count(stage, o, total)
        if park:
            assert tuple(float(o.state[key][0]) for key in ("x", "y", "theta")) == PARKED
            assert env0[3] == 1 and env0[6] == 1, ("the parked pose: passes 1+2 refused, 3+4 merged", env0)
    assert g.max() == 255
    env.close()

    env, o = _start(map_name, park)  # one tc_step_multi call
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
    torch.cuda.synchronize()
    for k in range(K):
        o.step(cc[k].astype(np.float64), man[k])
        assert np.array_equal(roll["cte"][k].cpu().numpy().view(np.int64), o.info["cte"].view(np.int64)), ("cte of step", k)
        g = roll["obs"][k].cpu().numpy().reshape(N, -1)
        bad = np.flatnonzero((g != o.obs).any(axis=1))
        assert bad.size == 0, ("tc_step_multi", map_name, merge, "step", k, "envs", bad[:8])
    env.close()

    print(map_name, "merge", merge, "pairs 1+2 / 3+4: empty, one list, merged, refused:", total[:4].tolist(), total[4:].tolist())
    assert total[2] + total[6] > 0, ("no frame of the run merges a pair", total)
    if park:
        assert total[3] >= K, total
