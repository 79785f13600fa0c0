"""The generated big maps (tests/big_maps.py) without a GPU: every case gets exactly the plan it is named for, the
camera stage's LDS layout of that plan is sound, and the oracle's rollout under the GPU test's own reset and actions
draws frames worth comparing -- so that tests/test_gpu_big_map_fuzz.py cannot go vacuous when the generator changes.
"""
import numpy as np
import pytest

import big_maps as bm
import cull_shim
import orc
from test_plan_cpu import _expect_failure, component_labels

CASE_SEEDS = [(name, k) for name in bm.CASES for k in range(bm.N_SEEDS)]


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def test_the_cases_cover_the_table():
    """one case at least for every row of the plan table and every frame kernel"""
    plans = [bm.case_map(name)[1] for name in bm.CASES]
    assert {(p["scheme"], p["kvar"], p["kframe"]) for p in plans} >= {
        ("single", 5, 5), ("single", 8, 8), ("layers", 9, 9), ("components", 9, 516), ("components", 9, 9), ("single", 13, 13)}
    assert max(p["n_layers"] for p in plans) == bm.MAX_LAYERS
    assert set(bm.SWITCH_CASES) <= set(bm.CASES)
    assert sum(c["fmt"] == "rgb" for c in bm.CASES.values()) == 2
    assert sum(c["res"][1] % 32 != 0 for c in bm.CASES.values()) == 1


@pytest.mark.parametrize("name,k", CASE_SEEDS)
def test_case_gets_the_plan_it_is_named_for(name, k):
    case = bm.CASES[name]
    mj, plan = bm.case_map(name, k)
    want = case["want"]
    assert bm.plan_misses(bm.expected_plan(mj, cam_group=case["cam_group"]), want) == []
    assert plan["total_nodes"] < 3000 and plan["n_layers"] <= bm.MAX_LAYERS
    big = max(plan["total_nodes"], plan["total_edges"])
    # the decisions around the planners, from the table: size classes, and groups only beyond 512
    assert (plan["kvar"] == 5) == (big <= 320) and (plan["kvar"] == 8) == (320 < big <= 512)
    assert (plan["scheme"] == "single") == (plan["n_groups"] == 1)
    if plan["scheme"] != "single":
        assert big > 512 and 2 <= plan["n_groups"] <= bm.MAX_GROUPS
        assert max(plan["cap_n"], plan["cap_e"]) <= (case["cam_group"] if plan["scheme"] == "components" else bm.LAYER_CAP)
    assert (plan["kframe"] == 516) == (plan["scheme"] == "components" and max(plan["cap_n"], plan["cap_e"]) <= 320)
    # the switches of the GPU test move the plan as the table says
    off = bm.expected_plan(mj, cam_group=case["cam_group"], groups=False)
    assert off["scheme"] == "single" and off["kvar"] == (plan["kvar"] if big <= 512 else 13)
    whole = bm.expected_plan(mj, cam_group=0)
    assert whole["scheme"] in ("single", "layers") and (whole["scheme"] == "layers") == (plan["scheme"] != "single")
    # why a map beyond 512 did not get component groups, worked out from its component sizes alone
    if "why" in want:
        _, _, edges = bm.graph_of_json(mj)
        assert _expect_failure(edges, component_labels(plan["total_nodes"], edges), case["cam_group"]) == want["why"]
    elif plan["scheme"] == "components":
        _, _, edges = bm.graph_of_json(mj)
        assert _expect_failure(edges, component_labels(plan["total_nodes"], edges), case["cam_group"]) is None


@pytest.mark.parametrize("name,k", CASE_SEEDS)
def test_camera_lds_layout(name, k):
    """plan_cam_lds for the case's caps: within a workgroup's 160 KB, buffers in order, 16-byte aligned, none
    overlapping -- with phase B's one double per node of the whole map aliased over the node buffer"""
    plan = bm.case_map(name, k)[1]
    L, cn, ce, tn = plan["lds"], plan["cap_n"], plan["cap_e"], plan["total_nodes"]
    assert L["total"] + bm.LIVE_BYTES <= bm.LDS_LIMIT
    assert L["off_p"] == 0 and all(L[key] % 16 == 0 for key in L)
    assert L["off_flg"] - L["off_p"] >= max(3 * cn * 8, tn * 8)
    assert L["off_list"] - L["off_flg"] >= cn
    assert L["off_cnt"] - L["off_list"] >= 4 * max(2 * ce, cn) + 16
    assert L["total"] - L["off_cnt"] >= 6 * 4
    if "min_lds" in bm.CASES[name]["want"]:
        assert L["total"] > bm.CASES[name]["want"]["min_lds"]


@pytest.fixture(scope="module")
def cull_lib(tmp_path_factory):
    return cull_shim.build_shim(tmp_path_factory.mktemp("tc_cull_big"))


@pytest.mark.parametrize("name,k", CASE_SEEDS)
def test_oracle_rollout_is_worth_comparing(name, k, tmp_path, cull_lib):
    """64 envs x 12 steps on the oracle alone, reset and actions as in the GPU test"""
    from oracle_backend import OracleVecEnv
    case = bm.CASES[name]
    plan = bm.case_map(name, k)[1]
    cfg = bm.case_config(name, k, tmp_path / "m.json")
    env = OracleVecEnv(cfg, num_envs=bm.N_ENVS, autoreset=True, spawn_queue_len=4)
    env.reset(seed=bm.case_seed(name, k))
    cc, man = bm.case_actions(name, k)
    frames = nonempty = 0
    drawn = np.zeros(plan["n_layers"], dtype=np.int64)
    for t in range(bm.N_STEPS):
        env.step({"car_control": cc[t], "maneuver": man[t]})
        for i in range(bm.N_ENVS):
            seg, _ = env._o.segments(i)
            frames += 1
            nonempty += len(seg) > 0
            drawn += np.bincount(seg[:, 0], minlength=plan["n_layers"])
    assert 2 * nonempty >= frames, (name, k, "mostly empty frames", nonempty, frames)
    assert (drawn > 0).all(), (name, k, "layers never drawn", np.flatnonzero(drawn == 0))
    for g in range(plan["n_groups"]):
        assert drawn[plan["l0"][g]:plan["l1"][g]].sum() > 0, (name, k, "camera group draws nothing", g)
    if "empty_frac" in case["want"]:
        assert frames - nonempty >= case["want"]["empty_frac"] * frames, (name, k, "too few empty frames", frames - nonempty, frames)
    if case["want"].get("cull"):
        # the whole-frame cull is on for this map and camera: H1-H3 of tc_cull.h hold (a table was planned, a cover found)
        cull = cull_shim.Cull(cull_lib, env.map, env.camera)
        assert cull.on and cull.nx > 0 and cull.lmax <= env.camera.max_range - 1e-3
        st = env._o.state
        assert cull.empty(st["x"], st["y"], st["theta"]).any(), "no pose of the last step is culled"
