"""Big-map fuzz: the grouped and windowed camera paths of the HIP library vs the CPU oracle on generated maps.

tests/test_gpu_map_fuzz.py covers arbitrary topologies on small maps, which almost always run the camera stage as one
register-cached group (K = 5 / 8).  The maps here (tests/big_maps.py: rings with gaps, dashes, interleaved / duplicate /
zero-length edges, self-loops, isolated nodes, layers with more edges than nodes, up to 16 layers, 320 .. 2 970 nodes)
sit on every boundary and branch of tc_env_create's plan: K = 5 | 8 | groups, groups of whole layers | of connected
components (renumbered camera copy, groups that start inside a layer or span several, frame kernel 516 | 9), and the
K = 13 windowed loops (by nodes, by edges only, four node windows and more than 48 KB of LDS).  tests/test_big_maps_cpu.py
holds each case to the plan it is named for and to frames that show the lines, so a pass here is not vacuous.

Per case, N = 64 envs with autoreset and a spawn queue of 4: launch_info and lds_bytes must match the plan worked out on
the host; then reset, 12 single steps (frames compared on every step) and one 12-step tc_step_multi call with a full
rollout, all bit-identical to the oracle (portable math).  Three cases are repeated under the switches that move the plan
or the kernels.  TC_BIG_FUZZ_SEEDS=n runs n maps per case (default 1; the CPU tests follow).
"""
import numpy as np
import pytest

import big_maps as bm
import orc
from test_gpu_bench_shapes import run_case
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

R_OFF_BITS = 6784  # R_OFF_BITS_OF(RB_MAX): the raster stage's tables in front of its band


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def check_creation(env, plan, case, fuse=True, env_grouped=True):
    """the handle took the path the plan names: kernels and K of a single step and of a 12-step call, LDS of a workgroup"""
    for steps in (1, bm.N_STEPS):
        kvar, kernel = bm.expected_launch(plan, steps, fuse=fuse, env_grouped=env_grouped)
        info = env.launch_info(steps)
        assert (info["kvar"], info["kernel"]) == (kvar, kernel), (steps, info, plan["scheme"], plan["kframe"])
        assert info["fused"] == (kernel == "tc_step_kernel")
    if plan["kframe"] == 516 and fuse:
        assert env.launch_info(1)["kvar"] == 5, "the fused kernel of a component-grouped map is the K = 5 one"
    # a workgroup's LDS: the camera stage's buffers for the plan's caps (plan_cam_lds) or the raster stage's tables and one
    # band of bit-planes, whichever is more, and the parked env state behind them
    cam = plan["lds"]["total"]
    H, W = case["res"]
    raster = R_OFF_BITS + -(-min(H * plan["n_layers"] * -(-W // 32) * 4, 16384) // 16) * 16
    assert cam + bm.LIVE_BYTES <= env.lds_bytes <= max(cam, raster) + bm.LIVE_BYTES, (env.lds_bytes, cam, raster)
    if "min_lds" in case["want"] and plan["scheme"] == "single":
        assert env.lds_bytes > case["want"]["min_lds"]


def run_big(name, k, tmp_path, plan=None, **switches):
    case = bm.CASES[name]
    if plan is None:
        plan = bm.case_map(name, k)[1]
    cfg = bm.case_config(name, k, tmp_path / "m.json")
    cc, man = bm.case_actions(name, k)
    N, K = bm.N_ENVS, bm.N_STEPS
    label = f"{name}/{k}"

    def single_steps(env, o):
        check_creation(env, plan, case, **switches)
        assert env.n_classes == plan["n_layers"]
        assert_same(env, o, env.n_classes, label=f"{label} reset")
        for t in range(K):
            o.step(cc[t].astype(np.float64), man[t], flags=orc.F_AUTORESET)
            env.step({"car_control": cc[t], "maneuver": man[t]})
            assert_same(env, o, env.n_classes, label=f"{label} step {t}")
            assert np.array_equal(env._aux["needs_reset"].cpu().numpy(), o.needs_reset)
        assert int(env.out["obs"].max()) > 0

    def multi_actions(n, steps, seed):
        return torch.from_numpy(cc[K:K + steps]).cuda(), torch.from_numpy(man[K:K + steps]).cuda()

    run_case(cfg, None, None, N, K, seed=bm.case_seed(name, k), actions=multi_actions, spawn_queue_len=4, threads=8, label=label,
             before=single_steps)


@pytest.mark.parametrize("name,k", [(name, k) for name in bm.CASES for k in range(bm.N_SEEDS)])
def test_big_map_rollout(name, k, tmp_path, monkeypatch):
    if bm.CASES[name]["cam_group"] != bm.CAM_GROUP:
        monkeypatch.setenv("TC_CAM_GROUP", str(bm.CASES[name]["cam_group"]))
    run_big(name, k, tmp_path)


SWITCHES = [("TC_FUSE", "0"), ("TC_GROUPS", "0"), ("TC_CAM_GROUP", "0"), ("TC_CAM_GROUP", "200"), ("TC_CAM_GROUP", "576"),
            ("TC_ENV_GROUPED", "0")]


@pytest.mark.parametrize("switch,value", SWITCHES)
@pytest.mark.parametrize("name", bm.SWITCH_CASES)
def test_big_map_switches(name, switch, value, tmp_path, monkeypatch):
    """the same rollout with a switch that moves the plan (TC_GROUPS, TC_CAM_GROUP) or the kernels (TC_FUSE: simulate and
    raster launches; TC_ENV_GROUPED: one wavefront per env in K-step calls); the plan is worked out for the switch"""
    monkeypatch.setenv(switch, value)
    case = bm.CASES[name]
    mj, _ = bm.case_map(name, 0)
    plan = bm.expected_plan(mj, cam_group=int(value) if switch == "TC_CAM_GROUP" else case["cam_group"], groups=(switch, value) != ("TC_GROUPS", "0"))
    run_big(name, 0, tmp_path, plan=plan, fuse=switch != "TC_FUSE", env_grouped=switch != "TC_ENV_GROUPED")
